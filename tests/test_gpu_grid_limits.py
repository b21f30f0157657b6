"""Every device launch past its 65535 grid-dimension limit, on the MI355X.

Some twenty launch sites put a row, polynomial or item count into grid dimension y or z, clamp it to 65535 and cover the rest with a stride loop in
the kernel or a slicing loop on the host; three entry-point families have no loop and refuse a batch above 65535, so 65535 itself must work.  The
limits count rows and items, not coefficients: every case runs at N = 16 (grid_cases.N), with 2 or 4 limbs (never a count that divides
65535 = 3 x 5 x 17 x 257: the row one stride later must land on another limb), at the smallest batch that puts the clamped dimension about 70 past the
limit.  Each case makes the three checks of grid_cases.run: the boundary items against an independent reference, EVERY item word for word against
the same call in chunks of 1024 items, and the footprint (a sentinel item behind every output, const operands unchanged).

troyhip_create_galois_keys is left out: its row count passes 65535 only with thousands of distinct Galois elements, which needs a ring far too large
for a test of seconds.  The refusal of a batch of 65536 by the capped entry points is tested in test_gpu_encode.py, test_gpu_encrypt.py,
test_gpu_keygen.py and test_gpu_noise.py and stays there.

Measured on the MI355X when the file was added: 32 cases in 2.3 s (tests/test_gpu_lazy.py: 1.7 s); the slowest, the 16-limb VALU multiply, 0.21 s
against a median of 0.03 s.  Sensitivity, shown once on scratch builds in which one loop ran its first iteration only (a `break` ending its body):
ew_kernel -- "add: item 16383 of 16402 differs from the reference"; tensor_kernel -- "multiply 2x2: item 65535 of 65605"; the slice loop of
launch_behz2_extend -- "multiply 2x2: item 32767 of 65605"; each the first item of the second stride or slice, each in the boundary set."""
import numpy as np
import pytest

import grid_cases as G
from grid_cases import BFV, CKKS, LIMIT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api.KernelProvider.lib()


BITS4 = {BFV: [45, 40, 40, 40, 45], CKKS: [50, 40, 40, 40, 50]}  # K = 5: levels of 4 and of 2 limbs
BITS2 = {BFV: [45, 40, 45], CKKS: [50, 40, 50]}                  # K = 3: 2 limbs


# ---------------------------------------------------------------- element-wise kernels through row_grid (grid y = rows)
@pytest.mark.parametrize("limbs", [2, 4])
@pytest.mark.parametrize("scheme", [BFV, CKKS], ids=["bfv_coeff", "ckks_ntt"])
@pytest.mark.parametrize("op", ["add", "sub", "negate"])
def test_ew_kernel_past_the_row_limit(op, scheme, limbs, lib):
    """poly.hip ew_kernel<0> (add), <1> (sub), <2> (negate) via row_grid: grid y = rows = batch x 2 x limbs, `row += gridDim.y`.  BFV in coefficient
    form and CKKS in NTT form: the kernel is the same, the LimbMap differs.  Reference: exact integers.  (ew_kernel<3>, the dyadic product, is
    launched with the rows of one secret-key power only -- `limbs` rows -- and cannot reach the limit; mul_plain_kernel is the product that can.)"""
    G.require_counts(limbs, 2 * limbs)
    batch = G.batch_past(2 * limbs)
    rows = batch * 2 * limbs
    assert LIMIT + 50 <= rows <= LIMIT + 100
    G.check_ew(G.setup(scheme, BITS4[scheme]), op, limbs, batch, seed=100 * limbs + scheme)


@pytest.mark.parametrize("plain", ["shared", "per_item"])
def test_mul_plain_kernel_past_the_row_limit(plain, lib):
    """poly.hip mul_plain_kernel via row_grid, rows = batch x 2 x limbs past 65535.  shared: troyhip_multiply_plain_ntt (CKKS, 4 limbs, one plaintext,
    rows_per_item = 0; exact integers).  per_item: troyhip_multiply_plain with one coefficient-form plaintext per item (BFV, 2 limbs,
    plain_batch_stride = N, so the plaintext pointer is recomputed per row from row / rows_per_item; the oracle item by item)."""
    limbs = 4 if plain == "shared" else 2
    G.require_counts(limbs, 2 * limbs)
    batch = G.batch_past(2 * limbs)
    assert LIMIT + 50 <= batch * 2 * limbs <= LIMIT + 100
    if plain == "shared":
        G.check_mul_plain_shared(G.setup(CKKS, BITS4[CKKS]), limbs, batch, seed=310)
    else:
        G.check_mul_plain_per_item(G.setup(BFV, BITS2[BFV]), limbs, batch, seed=320)


def test_mul_scalar_kernel_past_the_row_limit(lib):
    """poly.hip mul_scalar_kernel via row_grid: troyhip_divide_by_poly_modulus_degree with a multiplier other than 1, rows = batch x 2 x 4; the
    per-limb scalar is looked up per row.  Reference: exact integers."""
    limbs = 4
    G.require_counts(limbs, 2 * limbs)
    batch = G.batch_past(2 * limbs)
    assert LIMIT + 50 <= batch * 2 * limbs <= LIMIT + 100
    G.check_mul_scalar(G.setup(BFV, BITS4[BFV]), limbs, batch, seed=330)


# ---------------------------------------------------------------- grid z = batch
def test_mul_plain_acc_kernel_past_the_item_limit(lib):
    """poly.hip mul_plain_acc_kernel: troyhip_multiply_plain_accumulate, count = 3, CKKS, grid z = batch, `b += gridDim.z`.  Exact integers."""
    limbs = 2
    G.require_counts(limbs)
    batch = G.batch_past()
    assert LIMIT + 50 <= batch <= LIMIT + 100
    G.check_mul_plain_acc(G.setup(CKKS, BITS2[CKKS]), limbs, batch, seed=340)


def test_galois_ntt_kernel_past_the_item_limit(lib):
    """poly.hip galois_ntt_kernel: troyhip_apply_galois on NTT-form CKKS ciphertexts under a key from synth.uniform_kswitch_key, grid z = batch.  The
    key-switch kernels use flat grids; the oracle on the boundary set covers the whole call."""
    limbs = 2
    G.require_counts(limbs)
    batch = G.batch_past()
    assert LIMIT + 50 <= batch <= LIMIT + 100
    G.check_apply_galois(G.setup(CKKS, BITS2[CKKS]), limbs, batch, seed=350)


@pytest.mark.parametrize("family", ["fp", "mfma", "valu"])
def test_tensor_kernel_and_behz_slices_past_the_limits(family, lib):
    """BFV multiply 2 x 2 into a fresh dense destination: poly.hip tensor_kernel<2,2> in both bases (grid z = batch) and the host slice loops
    `p0 += 65535` of the extend and the floor / Shenoy-Kumaresan launchers -- behz3.hip (fp: launch_behz3_extend / _floor_sk), behz2.hip (mfma:
    launch_behz2_extend / _floor_sk), behz.hip (valu: launch_behz_extend / _floor_sk).  The family is selected by limb count and prime width as in
    test_behz_kernel_family_by_base and asserted with the same counters.  fp, mfma: batch past 65535, so polys = 2 batch per operand (three extend
    slices, the last short) and 3 batch in the product (four floor slices).  valu: 16 limbs, the smallest batch with two extend slices (polys
    just past 65535); its z loop is covered by the other two.  Reference: the oracle, item by item."""
    S = G.setup(BFV, G.BITS[family], tbits=14)
    limbs = S.ctx.first_limbs
    assert limbs == {"fp": 2, "mfma": 4, "valu": 16}[family]
    G.require_counts(limbs)
    if family == "valu":
        batch = G.batch_past(2)
        assert LIMIT < 2 * batch <= LIMIT + 100 and 3 * batch > LIMIT
    else:
        batch = G.batch_past()
        assert LIMIT + 50 <= batch <= LIMIT + 100 and 2 * batch > 2 * LIMIT and 3 * batch > 3 * LIMIT
    delta = G.check_multiply(S, 2, 2, batch, seed=400 + limbs)
    e = G.FAMILY_INDEX[family]
    assert delta[e] >= 2 and sum(delta) == delta[e], (family, delta)


@pytest.mark.parametrize("sa,sb", [(2, 3), (4, 2)])
def test_tensor_kernel_other_sizes_past_the_item_limit(sa, sb, lib):
    """2 x 3: poly.hip tensor_kernel<2,3>, grid z = batch past 65535 (and the BEHZ slices at 2, 3 and 4 polynomials per item).  4 x 2:
    tensor_any_kernel, a flat grid, as the control.  BFV, 2 limbs; the oracle item by item."""
    S = G.setup(BFV, G.BITS["fp"], tbits=14)
    limbs = S.ctx.first_limbs
    G.require_counts(limbs)
    batch = G.batch_past()
    assert LIMIT + 50 <= batch <= LIMIT + 100
    G.check_multiply(S, sa, sb, batch, seed=450 + sa)


def test_hoist_lt_base_kernel_past_the_item_limit(lib):
    """poly.hip hoist_lt_base_kernel: troyhip_galois_plain_sum_hoisted with three elements, one of them element 1, grid z = batch,
    `b += gridDim.z`; default scratch limit, ONE slab, so the kernel saw the whole batch.  Reference: the exact host model of hoist_lt_cases."""
    S = G.setup(BFV, BITS2[BFV])
    limbs = S.ctx.first_limbs
    G.require_counts(limbs)
    batch = G.batch_past()
    assert LIMIT + 50 <= batch <= LIMIT + 100
    assert G.check_hoist_lt(S, limbs, batch, seed=500) == 1


# ---------------------------------------------------------------- the samplers' and the key generator's row loops
def _enc_setup(bits):
    import enc_cases
    return enc_cases.Setup.from_cfg(dict(scheme=BFV, N=G.N, bits=bits, tbits=10))


def test_enc_pk_product_kernel_past_the_row_limit(lib):
    """sampler.hip enc_pk_product_kernel: troyhip_encrypt at the first level of K = 4 (3 data limbs, so el = 4 with the special prime), grid y = rows
    = batch x 2 x el, the row decomposed as row % el, (row / el) & 1, row / (2 el).  Item i against troyhip_host_encrypt with item i's seed."""
    ES = _enc_setup([45, 40, 40, 45])
    el = ES.ctx.first_limbs + 1
    G.require_counts(el, 2 * el)
    batch = G.batch_past(2 * el)
    assert LIMIT + 50 <= batch * 2 * el <= LIMIT + 100
    G.check_encrypt(ES, "pk", ES.ctx.first_limbs, batch, seed=600)


def test_enc_sk_combine_kernel_past_the_row_limit(lib):
    """sampler.hip enc_sk_combine_kernel: troyhip_encrypt_symmetric at 4 limbs, grid y = rows = batch x limbs.  Item i against
    troyhip_host_encrypt_symmetric with item i's seed."""
    ES = _enc_setup(BITS4[BFV])
    limbs = ES.ctx.first_limbs
    G.require_counts(limbs)
    batch = G.batch_past(limbs)
    assert LIMIT + 50 <= batch * limbs <= LIMIT + 100
    G.check_encrypt(ES, "sk", limbs, batch, seed=610)


def _keygen_setup(bits):
    import keygen_cases
    return keygen_cases.Setup.from_cfg(dict(scheme=BFV, N=G.N, bits=bits, tbits=10))


def test_key_combine_kernel_past_the_row_limit(lib):
    """keygen.hip key_combine_kernel: troyhip_keygen with K = 4, grid y = rows = batch x K.  Item i against troyhip_host_keygen with item i's seed."""
    KS = _keygen_setup([45, 40, 40, 45])
    G.require_counts(KS.K)
    batch = G.batch_past(KS.K)
    assert LIMIT + 50 <= batch * KS.K <= LIMIT + 100
    G.check_keygen(KS, batch, seed=620)


# ---------------------------------------------------------------- the top of the capped range: batch = 65535 exactly, no loop behind it
def test_batch_encode_decode_at_the_cap(lib):
    """encoder.hip bfv_encode_scatter_kernel, bfv_decode_load_kernel, bfv_decode_gather_kernel (b = blockIdx.y) and the transforms between them:
    troyhip_batch_encode / _decode at batch = 65535, N = 16 (every case of this file uses the one ring).  Item i against the host forms."""
    import encode_cases as EC
    G.check_batch_encode(EC.context(dict(scheme=BFV, N=G.N, bits=BITS2[BFV], tbits=10)), LIMIT, seed=700)


def test_ckks_encode_decode_at_the_cap(lib):
    """encoder.hip ckks_enc_lds_kernel, ckks_dec_garner_kernel, ckks_dec_lds_kernel (b = blockIdx.y): troyhip_ckks_encode / _decode at batch = 65535,
    N = 16, 2 limbs.  Item i against the host forms, doubles as bit patterns."""
    import encode_cases as EC
    G.check_ckks_encode(EC.context(dict(scheme=CKKS, N=G.N, bits=BITS2[CKKS], tbits=0)), 2, LIMIT, seed=710)


@pytest.mark.parametrize("form", ["pk", "sk"])
def test_encrypt_at_the_cap(form, lib):
    """sampler.hip: the sampling kernels of troyhip_encrypt (pk) / troyhip_encrypt_symmetric (sk) with b = blockIdx.y, at batch = 65535, 2 limbs.
    Item i against the host form with item i's seed."""
    ES = _enc_setup(BITS2[BFV])
    G.check_encrypt(ES, form, ES.ctx.first_limbs, LIMIT, seed=720 + len(form))


def test_keygen_at_the_cap(lib):
    """sampler.hip / keygen.hip: troyhip_keygen at batch = 65535, K = 2.  Item i against troyhip_host_keygen with item i's seed."""
    G.check_keygen(_keygen_setup([45, 45]), LIMIT, seed=730)


def test_noise_budget_at_the_cap(lib):
    """noise.hip noise_garner_kernel (b = blockIdx.y) and noise_item_kernel (b = blockIdx.x): troyhip_noise_budget with norms at batch = 65535 on
    ciphertexts troyhip_encrypt made, so the budgets are real.  Item i against troyhip_host_noise_budget."""
    import enc_cases
    import noise_cases
    NS = noise_cases.Setup(dict(scheme=BFV, N=G.N, bits=BITS2[BFV], tbits=10))
    ES = enc_cases.Setup(BFV, G.N, NS.primes, NS.t, key_seed=noise_cases.KEY_SEED)
    assert np.array_equal(ES.sk, NS.sk)
    limbs = NS.ctx.first_limbs
    cts = G.check_encrypt(ES, "pk", limbs, LIMIT, seed=740)
    budgets = G.check_noise_budget(NS, cts, limbs, LIMIT)
    assert budgets.min() > 0 and len(set(budgets.tolist())) > 1, "fresh encryptions: positive budgets that differ between items"
