"""The conditioning stages of `extract` and the truncated minimum-norm least squares on the MI355X (mtip_op_cc_lowpass_q,
mtip_op_cc_harmonic_filter, mtip_op_cc_binned_mean, csrc/k_extract_cond.h; mtip_op_cc_lstsq_deg2_minnorm, csrc/k_extract_lsq.h;
extract.modify_masked_cross_correlation): the cases of tests/cccond_cases.py against scipy's sosfilt, numpy's rfft / irfft, a
longdouble masked mean, the reference's own outputs (G30), numpy.linalg.lstsq and a longdouble minimum-norm solution."""
import pytest

import cccond_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden_cond():
    return DC.load_golden()


# n_q 5 and 70 (more than one workgroup row, a walk that is no multiple of the load depth), n_delta 64 and 70 (a lane tail)
@pytest.mark.parametrize('nq,nd,section,subtract', [(5, 64, 'order1', False), (5, 70, 'biquad', True), (70, 64, 'biquad', False),
                                                    (70, 70, 'order1', True), (5, 64, 'biquad', False), (5, 70, 'order1', False),
                                                    (70, 64, 'order1', True), (70, 70, 'biquad', False)])
def test_lowpass_scipy(nq, nd, section, subtract):
    DC.check_lowpass(None, nq, nd, section, subtract)


@pytest.mark.parametrize('label', list(DC.HARMONIC_SHAPES))
def test_harmonic_filter_numpy(label):
    DC.check_harmonic(None, label)


@pytest.mark.parametrize('label', list(DC.BINNED_SHAPES))
def test_binned_mean_longdouble(label):
    DC.check_binned(None, label)


def test_modify_golden(golden_cond):
    DC.check_modify_golden(golden_cond)


def test_bl_golden(golden_cond):
    DC.check_bl_golden(golden_cond)


def test_flow_golden(golden_cond):
    DC.check_flow_golden(golden_cond)


@pytest.mark.parametrize('label', DC.MINNORM_CASES)
def test_minimum_norm(label):
    DC.check_minnorm(None, label)


def test_minimum_norm_public():
    DC.check_minnorm_public(None)


def test_composition():
    DC.check_composition()


def test_limits():
    DC.check_limits()
