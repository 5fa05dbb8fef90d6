"""The route detector frames -> polar patterns on the MI355X (mtip_resample_*, mtip_correlate_add_detector, csrc/k_resample.h;
fxs/correlate.py Resampler / Correlator.add_detector): the cases of tests/resample_cases.py against the reference's own outputs
(G26) and an independent longdouble restatement of scipy.ndimage.map_coordinates.  Run with -s for the table device / bound."""
import pytest

import resample_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return RC.load_golden()


def test_device_golden(golden):
    RC.check_device_golden(golden)


@pytest.mark.parametrize('order', RC.ORDERS)
@pytest.mark.parametrize('shape', RC.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_shape_order(shape, order):
    RC.check_shape_order(None, shape, order)


@pytest.mark.parametrize('name', RC.SWITCH_NAMES)
def test_switches(name):
    for order in (2, 5):
        RC.check_switch(None, name, order)


def test_chunking():
    RC.check_chunking(None)


def test_batch_independence():
    RC.check_batch_independence(None)


def test_static_mask():
    RC.check_static_mask(None)


def test_host_and_device_input():
    RC.check_host_device(None)


def test_add_detector():
    RC.check_add_detector(None)


def test_raises():
    RC.check_raises(None)
