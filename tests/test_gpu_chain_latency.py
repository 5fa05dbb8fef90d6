"""MI355X: the Legendre synthesis of k_sht_chain / k_sht_inv_wide at the shapes where its padded records, uniform trip counts
and start-value queue can go wrong (tests/chain_latency_cases.py), against the oracle."""
import pytest

import chain_latency_cases as CL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('N,L', CL.TRANSFORM_CASES)
def test_transforms(N, L):
    CL.check_transforms(N, L, None)


def test_wide_two_theta_chunks():
    CL.check_wide_two_chunks(None)


@pytest.mark.parametrize('L', CL.UNIT_L)
def test_unit_coefficients(L):
    CL.check_unit_coefficients(L, None)


def test_fused_steps_ft_stab():
    CL.check_fused_steps_ft_stab(None)
