"""CPU pre-flight of `extract` on masked cross-correlation data (mtip_op_cc_prepare_masked, mtip_op_cc_lstsq_deg2,
csrc/k_extract_lsq.h; extract.masked_cross_correlation_to_deg2_invariant): the unchanged kernel source on the CPU emulator through the
cases of tests/test_gpu_ccmask.py, the large shapes at toy sizes."""
import os
import subprocess

import pytest

import ccmask_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden_masked():
    return MC.load_golden()


def test_prepare_golden(emul_lib, golden_masked):
    MC.check_prepare_golden(golden_masked, emul_lib)


def test_interpolation_scipy(emul_lib):
    MC.check_interpolation_scipy(emul_lib)


def test_lstsq_golden(emul_lib, golden_masked):
    MC.check_lstsq_golden(golden_masked, emul_lib)


def test_back_substitution_golden(emul_lib, golden_masked):
    MC.check_back_substitution_golden(golden_masked, emul_lib)


# (nq, L, odd orders assumed zero, n_delta, masked fraction): every register width, a partial block, blocks with a tail, 64 columns
@pytest.mark.parametrize('nq,L,zero_odd,nd,fraction', [(4, 8, True, 64, 1 / 16), (4, 8, False, 64, 1 / 16), (3, 32, True, 200, 1 / 25),
                                                       (3, 32, False, 200, 1 / 25), (2, 63, False, 256, 0.0), (2, 63, False, 256, 1 / 64)])
def test_lstsq_refined(emul_lib, nq, L, zero_odd, nd, fraction):
    MC.check_lstsq_refined(emul_lib, nq, L, zero_odd, nd, MC.periodic_mask(nq, nd, fraction), 'emulator')


def test_lstsq_random_masks(emul_lib):
    MC.check_lstsq_random_masks(emul_lib)


def test_limits(emul_lib):
    MC.check_limits(emul_lib)


def test_flow_golden(emul_lib, golden_masked):
    MC.check_flow_golden(golden_masked, emul_lib)


def test_end_to_end_correlator(emul_lib):
    MC.check_end_to_end_correlator(emul_lib)
