"""CPU pre-flight of the back-substitution modes memory_hungry, qqsym and psd (mtip_op_nearest_psd, mtip_op_cm_backsub,
csrc/k_extract_psd.h; extract.masked_cross_correlation_to_deg2_invariant): the unchanged kernel source on the CPU emulator through the
cases of tests/test_gpu_ccmodes.py at the same or smaller sizes, and the launch list of one psd call."""
import os
import subprocess

import pytest

import ccmodes_cases as QC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden_modes():
    return QC.load_golden()


# a single element, one pair, a tail of the 16 x 16 tile, two tiles per edge
@pytest.mark.parametrize('n', [1, 2, 5, 17, 33])
def test_nearest_psd(emul_lib, n):
    QC.check_nearest_psd(emul_lib, n)


@pytest.mark.parametrize('label', list(QC.SHAPES)[:3])
def test_modes_restatement(emul_lib, label):
    QC.check_modes_restatement(emul_lib, label)


def test_operator_golden(emul_lib, golden_modes):
    QC.check_operator_golden(golden_modes, emul_lib)


def test_flow_golden(emul_lib, golden_modes):
    QC.check_flow_golden(golden_modes, emul_lib)


def test_refusals(emul_lib):
    QC.check_refusals(emul_lib)


def test_launches(emul_lib):
    QC.check_launches(emul_lib)
