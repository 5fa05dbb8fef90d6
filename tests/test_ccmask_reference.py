"""CPU checks of `extract` on masked cross-correlation data that need no kernel: the host mask generators
(extract.cross_correlation_mask) and the numpy / scipy restatement of tests/ccmask_cases.py against the reference's own outputs
(G27, tests/golden/cc_masked.npz)."""
import pytest

import ccmask_cases as MC


@pytest.fixture(scope='module')
def golden_masked():
    return MC.load_golden()


def test_masks_golden(golden_masked):
    MC.check_masks_golden(golden_masked)


def test_restatement_golden(golden_masked):
    MC.check_restatement_golden(golden_masked)
