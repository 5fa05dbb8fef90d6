"""Cross-correlation -> B_l beyond 64 extracted orders on the MI355X (mtip_op_cc_to_deg2_wide, k_cc_deg2<HM> in csrc/k_extract.hip;
Engine.cc_to_deg2(wide=True), fxs/extract.py): the cases of tests/ccextract_wide_cases.py."""
import pytest

import ccextract_wide_cases as CW

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('nq,L,n_delta,zero_odd', CW.SHAPES)
def test_operator(nq, L, n_delta, zero_odd):
    CW.check_operator(None, nq, L, n_delta, zero_odd)


def test_dim2():
    CW.check_dim2(None)


def test_modify_flags():
    CW.check_modify_flags(None)


def test_same_kernel():
    CW.check_same_kernel(None)


def test_limits():
    CW.check_limits(None)


def test_masked_back_substitution():
    CW.check_masked_back_substitution(None)


def test_lstsq_refused():
    CW.check_lstsq_refused(None)


def test_flow_simulated():
    CW.check_flow_simulated(None)


def test_flow_synthetic():
    CW.check_flow_synthetic(None)


def test_into_loop():
    CW.check_into_loop(None)
