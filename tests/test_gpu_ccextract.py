"""The route cross-correlation -> B_l -> V_l on the MI355X (mtip_op_cc_to_deg2, csrc/k_extract.hip; fxs/extract.py): the cases of
tests/ccextract_cases.py against the reference's own outputs (G24) and, at sizes the fixture cannot hold, against the numpy
restatement that a CPU test holds to G24."""
import pytest

import ccextract_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden_cc():
    return CC.load_golden()


def test_operator_golden(golden_cc):
    CC.check_operator_golden(golden_cc)


@pytest.mark.parametrize('nq,L,n_delta,zero_odd', [(64, 32, 256, True), (64, 32, 256, False), (128, 32, 500, True), (256, 68, 512, True),
                                                   (512, 68, 1024, True)])
def test_operator_restatement(nq, L, n_delta, zero_odd):
    CC.check_operator_restatement(None, nq, L, n_delta, zero_odd)


def test_operator_device_tensor():
    CC.check_operator_restatement(None, 64, 32, 256, True, on_device_tensor=True)


def test_flow_golden(golden_cc):
    CC.check_flow_golden(golden_cc)


def test_end_to_end():
    CC.check_end_to_end(None, 128, 32, n_delta=1024)


def test_raises(golden_cc):
    CC.check_raises(golden_cc)
