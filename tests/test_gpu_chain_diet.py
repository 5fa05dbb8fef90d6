"""The leaner L = 32 instantiation of k_sht_chain on the MI355X through the cases of tests/chain_diet_cases.py: the two links on
seeded coefficients at the L32, REGTAB and RT shapes and 2 HIO + 2 ER fused steps at the L32 shape, bit for bit what the parent
commit's kernels gave on the MI355X (tests/golden/chain_bits.npz, keys gpu_*)."""
import pytest

import chain_diet_cases as DC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_transform_bits_as_the_parent(name):
    DC.check(DC.transform_results(name, None), 'gpu')


def test_fused_step_bits_as_the_parent():
    DC.check(DC.steps_results(None), 'gpu')


def test_l32_on_another_grid_falls_back():
    DC.check_fallback(None)
