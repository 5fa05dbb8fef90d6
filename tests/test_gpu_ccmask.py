"""`extract` on masked cross-correlation data on the MI355X (mtip_op_cc_prepare_masked, mtip_op_cc_lstsq_deg2,
csrc/k_extract_lsq.h; extract.masked_cross_correlation_to_deg2_invariant): the cases of tests/ccmask_cases.py against the reference's
own outputs (G27), against scipy's interp1d, and -- the least squares beyond the fixture -- against a longdouble-refined solution with
the bound taken from LAPACK's own error in the same case."""
import pytest

import ccmask_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden_masked():
    return MC.load_golden()


def test_prepare_golden(golden_masked):
    MC.check_prepare_golden(golden_masked)


def test_interpolation_scipy():
    MC.check_interpolation_scipy()


def test_lstsq_golden(golden_masked):
    MC.check_lstsq_golden(golden_masked)


def test_back_substitution_golden(golden_masked):
    MC.check_back_substitution_golden(golden_masked)


@pytest.mark.parametrize('label', list(MC.REFINED_SHAPES))
def test_lstsq_refined(label):
    MC.check_lstsq_shape(None, label)


def test_lstsq_random_masks():
    MC.check_lstsq_random_masks(None)


def test_limits():
    MC.check_limits()


def test_flow_golden(golden_masked):
    MC.check_flow_golden(golden_masked)


def test_end_to_end_correlator():
    MC.check_end_to_end_correlator()
