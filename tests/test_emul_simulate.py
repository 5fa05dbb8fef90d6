"""CPU pre-flight of the worker `simulate_ccd`: B_l -> C(q1, q2, Delta) (mtip_op_deg2_to_cc, csrc/k_simulate.h; fxs/simulate_ccd.py): the
unchanged kernel source on the CPU emulator through the cases of tests/test_gpu_simulate.py, the numpy restatements and the host tables
against the reference's own outputs (G28), and what only the emulator can see (the launch log, the NaN-filled output)."""
import os
import subprocess

import pytest

import simulate_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden():
    return SC.load_golden()


def test_restatement_golden(golden):
    SC.check_restatement_golden(golden)


def test_operator_golden(emul_lib, golden):
    SC.check_operator_golden(golden, emul_lib)


@pytest.mark.parametrize('dimensions', [3, 2])
@pytest.mark.parametrize('nq,L', SC.HARMONIC_SHAPES)
def test_bound_harmonics(emul_lib, nq, L, dimensions):
    SC.check_bound_harmonics(emul_lib, nq, L, dimensions)


@pytest.mark.parametrize('nq,L,n_delta', SC.LSTSQ_SHAPES)
def test_bound_lstsq(emul_lib, nq, L, n_delta):
    SC.check_bound_lstsq(emul_lib, nq, L, n_delta)


@pytest.mark.parametrize('stride', [1, 2])
def test_round_trip(emul_lib, stride):
    SC.check_round_trip(emul_lib, stride)


def test_flow(emul_lib, golden):
    SC.check_flow(golden, emul_lib)


def test_raises(emul_lib, golden):
    SC.check_raises(golden, emul_lib)


def test_overwrite_and_launches(emul_lib):
    SC.check_overwrite_and_launches(emul_lib)
