"""CPU pre-flight of the alignment and averaging operators (csrc/k_align.hip, csrc/k_average.hip): the unchanged kernel sources on
the CPU emulator through the cases of tests/align_cases.py at toy sizes, against the longdouble references of
tests/so3_reference.py (which tests/test_so3_reference.py holds to the exact Wigner sum and to rotated functions)."""
import os
import subprocess

import pytest

import align_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')

SO3_SIZES = [(6, 1, 2, None), (5, 4, 3, (1, 4)), (8, 10, 2, (7, 8))]
GRIDS = [(6, 4), (24, 10)]


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('spectrum', ['decay', 'flat'])
@pytest.mark.parametrize('N,L,B,shells', SO3_SIZES)
def test_correlation(emul_lib, N, L, B, shells, spectrum):
    AC.check_correlation(emul_lib, N, L, B, shells, spectrum)


@pytest.mark.parametrize('spectrum', ['decay', 'flat'])
@pytest.mark.parametrize('N,L,B,shells', SO3_SIZES)
def test_rotation(emul_lib, N, L, B, shells, spectrum):
    AC.check_rotation(emul_lib, N, L, B, spectrum)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('N,L', GRIDS)
def test_grid_stats(emul_lib, N, L, n):
    AC.check_grid_stats(emul_lib, N, L, n)


def test_grid_stats_nan(emul_lib):
    AC.check_grid_stats_nan(emul_lib)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('N,L', GRIDS)
def test_phase_ramp(emul_lib, N, L, n):
    AC.check_phase_ramp(emul_lib, N, L, n)


@pytest.mark.parametrize('N,L,n', [(6, 4, 1), (6, 4, 2), (6, 4, 8), (24, 10, 2)])
def test_combine(emul_lib, N, L, n):
    AC.check_combine(emul_lib, N, L, n)


@pytest.mark.parametrize('N,L', GRIDS)
def test_prtf(emul_lib, N, L):
    AC.check_prtf(emul_lib, N, L)
