"""CPU pre-flight of the correlate route at the lengths of mtip_correlate_create_ex with MTIP_CORRELATE_ANY_NPHI
(csrc/k_correlate_bs.h; ``Correlator(..., any_n_phi=True)``): the unchanged kernel source on the CPU emulator through the cases of
tests/test_gpu_correlate_anyphi.py at toy sizes, and what only the emulator can see (the launch logs)."""
import os
import subprocess

import pytest

import correlate_anyphi_cases as CA

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('name', list(CA.TOY) + ['grid_stride'])
def test_case(emul_lib, name):
    CA.check_case(emul_lib, name)


def test_shared_mask(emul_lib):
    CA.check_shared_mask(emul_lib)


def test_batch_independence(emul_lib):
    CA.check_batch_independence(emul_lib)


def test_partial_merge(emul_lib):
    CA.check_merge(emul_lib)


def test_finalize(emul_lib):
    CA.check_finalize(emul_lib)


def test_route_unchanged(emul_lib):
    CA.check_route_unchanged(emul_lib)


def test_max_mode(emul_lib):
    CA.check_max_mode(emul_lib)


def test_ok():
    CA.check_ok()


def test_raises(emul_lib):
    CA.check_raises(emul_lib)
