"""CPU pre-flight of the route cross-correlation -> B_l -> V_l (mtip_op_cc_to_deg2, csrc/k_extract.hip; fxs/extract.py, io.load_ccd):
the unchanged kernel source on the CPU emulator through the cases of tests/test_gpu_ccextract.py at toy sizes, the numpy restatement
against the reference's own outputs (G24), and what only the emulator can see (the launch log, the NaN-filled output)."""
import os
import subprocess

import pytest

import ccextract_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden_cc():
    return CC.load_golden()


def test_restatement_golden(golden_cc):
    CC.check_restatement_golden(golden_cc)


def test_load_ccd():
    CC.check_load_ccd()


def test_operator_golden(emul_lib, golden_cc):
    CC.check_operator_golden(golden_cc, emul_lib)


@pytest.mark.parametrize('nq,L,n_delta,zero_odd', [(64, 32, 256, True), (64, 32, 256, False), (128, 32, 500, True)])
def test_operator_restatement(emul_lib, nq, L, n_delta, zero_odd):
    CC.check_operator_restatement(emul_lib, nq, L, n_delta, zero_odd)


def test_flow_golden(emul_lib, golden_cc):
    CC.check_flow_golden(golden_cc, emul_lib)


def test_end_to_end(emul_lib):
    CC.check_end_to_end(emul_lib, 32, 8)


def test_raises(emul_lib, golden_cc):
    CC.check_raises(golden_cc, emul_lib)


def test_overwrite_and_launches(emul_lib):
    CC.check_overwrite_and_launches(emul_lib)
