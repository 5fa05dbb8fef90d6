"""The yardsticks of tests/resample_cases.py against each other, without any kernel: the numpy restatement of process_image 382-398
against the reference's own outputs (G26), scipy.ndimage.map_coordinates and the restatement against the longdouble reference at a
quarter of the device's bound, and read_raw_images."""
import pytest

import resample_cases as RC


@pytest.fixture(scope='module')
def golden():
    return RC.load_golden()


def test_restatement_golden(golden):
    RC.check_restatement_golden(golden)


@pytest.mark.parametrize('order', RC.ORDERS)
@pytest.mark.parametrize('shape', RC.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_scipy_and_restatement(shape, order):
    RC.check_reference_case(shape, order, 'all', 'float64')
    RC.check_reference_case(shape, order, 'masks', 'float32')


@pytest.mark.parametrize('name', RC.SWITCH_NAMES)
def test_switches(name):
    for order in (2, 5):
        RC.check_reference_case((37, 53), order, name, 'float64')


def test_overshoot_mask_exists():
    """the input of the device's raise test: a 0 / 1 mask whose cubic interpolant rounds to 2, by scipy as well"""
    import numpy as np
    mask, value = RC.overshoot_mask(12, 12, 3, 5, 5)
    assert value > 1.5 + 1e-6
    _, sm = RC.scipy_resample(np.ones((1, 12, 12)), mask[None], np.array([5.5]), np.array([5.5]), 3)
    assert sm[0, 0] == 2


def test_read_raw_images(tmp_path):
    RC.check_read_raw_images(tmp_path)
