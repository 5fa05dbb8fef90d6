"""The route patterns -> C(q1, q2, Delta) on the MI355X (mtip_correlate_*, csrc/k_correlate.h; fxs/correlate.py): the cases of
tests/correlate_cases.py against the reference's own outputs (G25) and, at sizes the fixture cannot hold, against the numpy
restatement (held to G25 by a CPU test) and an independent longdouble direct-sum correlation with exact integer pair counts."""
import pytest

import correlate_cases as CO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return CO.load_golden()


def test_device_golden(golden):
    CO.check_device_golden(golden)


@pytest.mark.parametrize('name', list(CO.CASES) + ['grid_stride'])
def test_case(name):
    CO.check_case(None, name)


def test_sparse_masks():
    CO.check_sparse(None)


def test_shared_mask():
    CO.check_shared_mask(None)


def test_batch_independence():
    CO.check_batch_independence(None)


def test_partial_merge():
    CO.check_merge(None)


def test_finalize():
    CO.check_finalize(None)


def test_device_tensor():
    CO.check_device_tensor(None)


def test_end_to_end():
    CO.check_end_to_end(None, P=400)            # (the emulator's 12 patterns leave a statistical error of order one)


def test_raises():
    CO.check_raises(None)
