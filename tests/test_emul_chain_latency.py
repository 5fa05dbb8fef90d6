"""CPU emulator twin of tests/test_gpu_chain_latency.py: the same cases (tests/chain_latency_cases.py) on the kernel sources
compiled for the host -- index, barrier and out-of-bounds mistakes show here before a GPU is involved."""
import os
import subprocess

import pytest

import chain_latency_cases as CL

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')


@pytest.fixture(scope='module')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.mark.parametrize('N,L', CL.TRANSFORM_CASES)
def test_transforms(emul_lib, N, L):
    CL.check_transforms(N, L, emul_lib)


def test_wide_two_theta_chunks(emul_lib):
    CL.check_wide_two_chunks(emul_lib)


@pytest.mark.parametrize('L', CL.UNIT_L)
def test_unit_coefficients(emul_lib, L):
    CL.check_unit_coefficients(L, emul_lib)


def test_fused_steps_ft_stab(emul_lib):
    CL.check_fused_steps_ft_stab(emul_lib)
