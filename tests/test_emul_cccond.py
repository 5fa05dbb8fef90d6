"""CPU pre-flight of the conditioning stages of `extract` and of the truncated minimum-norm least squares (mtip_op_cc_lowpass_q,
mtip_op_cc_harmonic_filter, mtip_op_cc_binned_mean, mtip_op_cc_lstsq_deg2_minnorm; csrc/k_extract_cond.h, csrc/k_extract_lsq.h): the
unchanged kernel source on the CPU emulator through the cases of tests/test_gpu_cccond.py at the same toy sizes, and the limits and
refusals."""
import os
import subprocess

import pytest

import cccond_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden_cond():
    return DC.load_golden()


@pytest.mark.parametrize('nq,nd,section,subtract', [(5, 64, 'order1', False), (5, 70, 'biquad', True), (70, 64, 'biquad', False),
                                                    (70, 70, 'order1', True), (5, 64, 'biquad', False), (5, 70, 'order1', False),
                                                    (70, 64, 'order1', True), (70, 70, 'biquad', False)])
def test_lowpass_scipy(emul_lib, nq, nd, section, subtract):
    DC.check_lowpass(emul_lib, nq, nd, section, subtract)


@pytest.mark.parametrize('label', list(DC.HARMONIC_SHAPES))
def test_harmonic_filter_numpy(emul_lib, label):
    DC.check_harmonic(emul_lib, label)


@pytest.mark.parametrize('label', list(DC.BINNED_SHAPES))
def test_binned_mean_longdouble(emul_lib, label):
    DC.check_binned(emul_lib, label)


def test_modify_golden(emul_lib, golden_cond):
    DC.check_modify_golden(golden_cond, emul_lib)


def test_bl_golden(emul_lib, golden_cond):
    DC.check_bl_golden(golden_cond, emul_lib)


def test_flow_golden(emul_lib, golden_cond):
    DC.check_flow_golden(golden_cond, emul_lib)


@pytest.mark.parametrize('label', DC.MINNORM_CASES)
def test_minimum_norm(emul_lib, label):
    DC.check_minnorm(emul_lib, label)


def test_minimum_norm_public(emul_lib):
    DC.check_minnorm_public(emul_lib)


def test_composition(emul_lib):
    DC.check_composition(emul_lib)


def test_limits(emul_lib):
    DC.check_limits(emul_lib)


def test_refusals(emul_lib):
    DC.check_refusals(emul_lib)
