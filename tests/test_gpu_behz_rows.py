"""The large-base matrix-core BEHZ kernels at every limb count that changes their shape (tests/behz_row_cases.py) on the MI355X, where the products
are v_mfma_i32_32x32x32_i8 and the launches carry the instances' names: behz2_extend_kernel<3 | 4> and behz2_floor_sk_kernel<3, 3 | 4, 4, true>."""
import pytest

import behz_row_cases as BR

_setups = {}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_api():
    from troy_amd import api
    api.KernelProvider.initialize(0)
    return api


@pytest.mark.parametrize("L", BR.LIMBS)
def test_behz_rows(L, gpu_api):
    BR.check(_setups, L)
