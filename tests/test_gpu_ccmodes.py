"""The back-substitution modes memory_hungry, qqsym and psd on the MI355X (mtip_op_nearest_psd, mtip_op_cm_backsub,
csrc/k_extract_psd.h; extract.masked_cross_correlation_to_deg2_invariant): the cases of tests/ccmodes_cases.py against the reference's
own outputs (G31), against numpy for the nearest PSD matrix, and beyond the fixture against the numpy restatement with the per-order
bound taken from the restatement's own two summation orders."""
import pytest

import ccmodes_cases as QC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden_modes():
    return QC.load_golden()


@pytest.mark.parametrize('n', QC.PSD_SIZES)
def test_nearest_psd(n):
    QC.check_nearest_psd(None, n)


@pytest.mark.parametrize('label', list(QC.SHAPES))
def test_modes_restatement(label):
    QC.check_modes_restatement(None, label)


def test_operator_golden(golden_modes):
    QC.check_operator_golden(golden_modes)


def test_flow_golden(golden_modes):
    QC.check_flow_golden(golden_modes)


def test_refusals():
    QC.check_refusals()
