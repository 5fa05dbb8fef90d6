"""CPU pre-flight of the median_mad radial pixel filter (csrc/k_ringfilter.h; ``Correlator(..., median_mad=True)``,
``correlate.ring_median_mad``): the unchanged kernel source on the CPU emulator through the cases of tests/test_gpu_ringfilter.py, and
the yardstick itself against numpy / scipy and against the reference's own functions (G29)."""
import os
import subprocess

import pytest

import ringfilter_cases as RF

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


def test_restatement_numpy_scipy():
    RF.check_restatement_numpy_scipy()


def test_restatement_golden():
    RF.check_restatement_golden(RF.load_golden())


@pytest.mark.parametrize('n_phi', RF.LENGTHS)
def test_operator(emul_lib, n_phi):
    RF.check_operator(emul_lib, n_phi)


def test_many_rows(emul_lib):
    RF.check_many_rows(emul_lib)


@pytest.mark.parametrize('name', list(RF.EQUIVALENCE))
def test_equivalence(emul_lib, name):
    RF.check_equivalence(emul_lib, name)


def test_device_golden(emul_lib):
    RF.check_device_golden(RF.load_golden(), emul_lib)


def test_add_detector(emul_lib):
    RF.check_add_detector(emul_lib)


def test_batch_independence(emul_lib):
    RF.check_batch_independence(emul_lib)


def test_settings_key(emul_lib):
    RF.check_settings_key(emul_lib)


def test_raises(emul_lib):
    RF.check_raises(emul_lib)
