"""The correlate route on the MI355X at the lengths of mtip_correlate_create_ex with MTIP_CORRELATE_GENERAL_NPHI
(csrc/k_correlate_mr.h; ``Correlator(..., general_n_phi=True)``): every case of tests/correlate_nphi_cases.py, 1536 (the default
settings' length), 1920, 2000 and 2048 among them, against the longdouble direct-sum correlation with exact integer pair counts."""
import pytest

import correlate_nphi_cases as CN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(CN.CASES) + ['grid_stride'])
def test_case(name):
    CN.check_case(None, name)


def test_shared_mask():
    CN.check_shared_mask(None)


def test_batch_independence():
    CN.check_batch_independence(None)


def test_partial_merge():
    CN.check_merge(None)


def test_finalize():
    CN.check_finalize(None)


def test_add_detector():
    CN.check_add_detector(None)


def test_end_to_end():
    CN.check_end_to_end(None, P=400)            # (the emulator's 12 patterns leave a statistical error of order one)


def test_flag_changes_nothing():
    CN.check_flag_changes_nothing(None)


def test_raises():
    CN.check_raises(None)


def test_default_settings():
    CN.check_default_settings(None)
