"""The correlate route on the MI355X at the lengths of mtip_correlate_create_ex with MTIP_CORRELATE_ANY_NPHI
(csrc/k_correlate_bs.h; ``Correlator(..., any_n_phi=True)``): every case of tests/correlate_anyphi_cases.py, 1046, 1256 (a ring of
200 pixels radius in phi_range's 'max' mode), 2042 and 2046 among them, against the longdouble direct-sum correlation with exact
integer pair counts."""
import pytest

import correlate_anyphi_cases as CA

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(CA.CASES) + ['grid_stride'])
def test_case(name):
    CA.check_case(None, name)


def test_shared_mask():
    CA.check_shared_mask(None)


def test_batch_independence():
    CA.check_batch_independence(None)


def test_partial_merge():
    CA.check_merge(None)


def test_finalize():
    CA.check_finalize(None)


def test_route_unchanged():
    CA.check_route_unchanged(None)


def test_max_mode():
    CA.check_max_mode(None)


def test_raises():
    CA.check_raises(None)
