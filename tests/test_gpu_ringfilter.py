"""The median_mad radial pixel filter on the MI355X (csrc/k_ringfilter.h: k_corr_stats_mad; ``mtip_op_ring_median_mad``,
``Correlator(..., median_mad=True)``): every case of tests/ringfilter_cases.py.  The operator against the sort-based restatement of
np.nanmedian / scipy.stats.median_abs_deviation, bit for bit; a filtered handle against an unfiltered one fed the restatement's
filtered patterns, bit for bit; the reference's own process_image (G29)."""
import pytest

import ringfilter_cases as RF

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n_phi', RF.LENGTHS)
def test_operator(n_phi):
    RF.check_operator(None, n_phi)


def test_many_rows():
    RF.check_many_rows(None)


@pytest.mark.parametrize('name', list(RF.EQUIVALENCE))
def test_equivalence(name):
    RF.check_equivalence(None, name)


def test_device_golden():
    RF.check_device_golden(RF.load_golden())


def test_add_detector():
    RF.check_add_detector(None)


def test_batch_independence():
    RF.check_batch_independence(None)


def test_settings_key():
    RF.check_settings_key(None)


def test_raises():
    RF.check_raises(None)
