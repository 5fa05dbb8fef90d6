"""CPU pre-flight of cross-correlation -> B_l beyond 64 extracted orders (mtip_op_cc_to_deg2_wide, k_cc_deg2<HM> in
csrc/k_extract.hip): the unchanged kernel source on the CPU emulator through the cases of tests/test_gpu_ccextract_wide.py, what only
the emulator can see (the launch log; the canary behind the staging buffer in dynamic LDS), and the Legendre table against mpmath."""
import os
import subprocess

import pytest

import ccextract_wide_cases as CW

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


def test_legendre_table():
    CW.check_legendre_table()


@pytest.mark.parametrize('nq,L,n_delta,zero_odd', CW.EMUL_SHAPES)
def test_operator(emul_lib, nq, L, n_delta, zero_odd):
    CW.check_operator(emul_lib, nq, L, n_delta, zero_odd)


def test_dim2(emul_lib):
    CW.check_dim2(emul_lib)


def test_modify_flags(emul_lib):
    CW.check_modify_flags(emul_lib)


def test_same_kernel(emul_lib):
    CW.check_same_kernel(emul_lib)


def test_limits(emul_lib):
    CW.check_limits(emul_lib)


def test_masked_back_substitution(emul_lib):
    CW.check_masked_back_substitution(emul_lib)


def test_lstsq_refused(emul_lib):
    CW.check_lstsq_refused(emul_lib)


def test_flow_synthetic(emul_lib):
    CW.check_flow_synthetic(emul_lib)
