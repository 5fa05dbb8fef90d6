"""The worker `simulate_ccd` on the MI355X: B_l -> C(q1, q2, Delta) (mtip_op_deg2_to_cc, csrc/k_simulate.h; fxs/simulate_ccd.py): the cases
of tests/simulate_cases.py against the reference's own outputs (G28), against a direct sum in extended precision with an a-priori bound
per element, and through the round trip with `extract`."""
import pytest

import simulate_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return SC.load_golden()


def test_operator_golden(golden):
    SC.check_operator_golden(golden)


@pytest.mark.parametrize('dimensions', [3, 2])
@pytest.mark.parametrize('nq,L', SC.HARMONIC_SHAPES)
def test_bound_harmonics(nq, L, dimensions):
    SC.check_bound_harmonics(None, nq, L, dimensions)


@pytest.mark.parametrize('nq,L,n_delta', SC.LSTSQ_SHAPES)
def test_bound_lstsq(nq, L, n_delta):
    SC.check_bound_lstsq(None, nq, L, n_delta)


@pytest.mark.parametrize('stride,on_device', [(1, False), (2, False), (2, True)])
def test_round_trip(stride, on_device):
    SC.check_round_trip(None, stride, on_device)


def test_flow(golden):
    SC.check_flow(golden)


def test_raises(golden):
    SC.check_raises(golden)
