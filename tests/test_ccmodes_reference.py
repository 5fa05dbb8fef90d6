"""CPU check that needs no kernel: the numpy restatement of the back-substitution modes memory_hungry, qqsym and psd
(tests/ccmodes_reference.py) against the reference's own outputs (G31, tests/golden/cc_backsub_modes.npz); the generator measured
0.0 for the modes and 1.1e-15 for the shifted eigh, the bound is 1e-13.  The fixture's inputs are the seeded ones of
ccmodes_cases.golden_inputs, and the cases of the device tests are not vacuous: every shape clips and differs from the plain mode."""
import numpy as np
import pytest

import ccmodes_cases as QC


@pytest.fixture(scope='module')
def golden_modes():
    return QC.load_golden()


def test_restatement_golden(golden_modes):
    QC.check_restatement_golden(golden_modes)


def test_reference_distance_recorded(golden_modes):
    # the reference's two implementations of the plain elimination agree to the bit on this data: the device may return one kernel's bits
    for name in ('s2', 's1'):
        assert float(golden_modes[f'G31_hungry_vs_back_substitution_{name}']) == 0.0
    assert np.any(golden_modes['G31_back_substitution_psd_s2_b'].imag)


@pytest.mark.parametrize('label', list(QC.SHAPES)[:3])
def test_cases_not_vacuous(label):
    QC.assert_not_vacuous(label)
