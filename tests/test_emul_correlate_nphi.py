"""CPU pre-flight of the correlate route at the lengths of mtip_correlate_create_ex with MTIP_CORRELATE_GENERAL_NPHI
(csrc/k_correlate_mr.h; ``Correlator(..., general_n_phi=True)``): the unchanged kernel source on the CPU emulator through the cases of
tests/test_gpu_correlate_nphi.py at toy sizes, and what only the emulator can see (the launch logs)."""
import os
import subprocess

import pytest

import correlate_nphi_cases as CN

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('name', list(CN.TOY) + ['grid_stride'])
def test_case(emul_lib, name):
    CN.check_case(emul_lib, name)


def test_shared_mask(emul_lib):
    CN.check_shared_mask(emul_lib)


def test_batch_independence(emul_lib):
    CN.check_batch_independence(emul_lib)


def test_partial_merge(emul_lib):
    CN.check_merge(emul_lib)


def test_finalize(emul_lib):
    CN.check_finalize(emul_lib)


def test_add_detector(emul_lib):
    CN.check_add_detector(emul_lib)


def test_end_to_end(emul_lib):
    CN.check_end_to_end(emul_lib)


def test_flag_changes_nothing(emul_lib):
    CN.check_flag_changes_nothing(emul_lib)


def test_near():
    CN.check_near()


def test_raises(emul_lib):
    CN.check_raises(emul_lib)


def test_default_settings(emul_lib):
    CN.check_default_settings(emul_lib)
